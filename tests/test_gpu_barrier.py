"""GPU: ``sit_barrier_energies`` and ``MergeSitesByBarrier`` against the numpy restatement (tests/barrier_ref.py, pinned to the
TRUE reference by tests/test_barrier_ref.py) and against the reference's goldens (tests/golden/barrier_known_answers.npz).

Energies are compared per image within ``1e-10 * sum |phi|`` of that image.  That is derived, not measured: a float64 sum of
``n_terms`` terms taken in another order errs by at most about ``n_terms * 2^-53 * sum |phi|``, and every case here keeps
``n_terms <= 1e5`` (asserted), so the bound is about ``1.1e-11 * sum |phi|``.  Pairs, codes, verdicts, the mergable matrix,
groups, trajectories, centres and site types are compared exactly.  The shapes are the smallest at which the kernel can go
wrong: S around the wave width and the LDS tile, n around the number of waves, one workgroup and many."""
import functools

import numpy as np
import pytest

from tests import barrier_ref as BR

pytestmark = pytest.mark.gpu

BG = BR.BarrierGoldens()
TOL = 1e-10
CELLS = {"cubic": BR.CUBIC, "cubic4": np.eye(3) * 4.0, "triclinic": BR.TRICLINIC, "small_triclinic": BR.SMALL_TRICLINIC}

# (cell, rc / smallest height, S, n, P, atoms given outside the cell)
RAW = [
    ("cubic", 0.45, 1, 3, 1, False),
    ("cubic", 0.45, 3, 3, 1, False),
    ("cubic", 0.45, 3, 3, 3, False),
    ("cubic", 0.45, 63, 4, 2, False),
    ("cubic", 0.45, 64, 5, 1, False),
    ("cubic", 0.45, 65, 67, 2, True),
    ("cubic", 0.45, "tile", 3, 1, False),
    ("cubic", 0.45, "tile+1", 20, 2, True),
    ("cubic", 0.45, 5, 3, 300, False),
    ("cubic4", 2.6, 1, 4, 1, False),
    ("cubic4", 2.6, 65, 5, 2, True),
    ("cubic4", 2.6, "tile+1", 3, 1, False),
    ("triclinic", 0.45, 65, 20, 2, True),
    ("triclinic", 0.3, "tile+1", 5, 1, False),
    ("small_triclinic", 1.4, 3, 5, 2, True),
]


def tile_size():
    from sitator_amd import _lib
    return _lib.barrier_plan(np.eye(3) * 10.0, 1.0)["tile"]


@functools.lru_cache(maxsize=None)
def raw_case(cell_name, factor, S, n, P, outside):
    """The inputs of one raw call and the restatement's answer, computed once."""
    if isinstance(S, str):
        S = tile_size() + (1 if S.endswith("+1") else 0)
    cell = CELLS[cell_name]
    rng = np.random.default_rng(1000 * S + 10 * n + P)
    rc = factor * BR.heights(cell).min()
    static = rng.uniform(0.0, 1.0, (S, 3)) @ cell
    if outside:
        static += rng.integers(-2, 3, (S, 3)).astype(np.float64) @ cell
    species = rng.integers(0, 2, S)
    eps, sigma = np.where(species == 1, 0.6, 1.0), np.where(species == 1, 0.8, 1.0) * rc / 3.0
    centers = rng.uniform(0.0, 1.0, (P + 1, 3)) @ cell
    pairs = np.stack([np.arange(P), np.arange(P) + 1], axis=1)
    points, codes = BR.driven_points(cell, centers, pairs, n)
    if P:                                                        # the first atom beside the first path, whatever S is
        static[0] = points[0, n // 2] + 0.3 * rc * np.array([0.6, 0.0, 0.8]) + (np.array([1.0, -2.0, 0.0]) @ cell if outside else 0.0)
    energies, abs_sums, n_terms = BR.path_energies(cell, static, eps, sigma, rc, points)
    threshold = float(np.median(np.max(energies, axis=1) - energies[:, 0])) if P else 1.0
    verdicts = np.array([BR.verdict(row, threshold) for row in energies], dtype=np.uint8).reshape(P, 3)
    return {"cell": cell, "static": static, "eps": eps, "sigma": sigma, "rc": rc, "centers": centers, "pairs": pairs, "n": n,
            "threshold": threshold, "codes": codes, "energies": energies, "abs_sums": abs_sums, "n_terms": n_terms,
            "verdicts": verdicts}


@pytest.fixture(scope="module")
def contexts():
    from sitator_amd import _lib
    made = {}

    def get(cell):
        key = np.asarray(cell, dtype=np.float64).tobytes()
        if key not in made:
            made[key] = _lib.HipContext(cell)
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def call(ctx, c, **over):
    a = dict(c, **over)
    return ctx.barrier_energies(a["static"], a["eps"], a["sigma"], a["rc"], a["centers"], a["pairs"], np.linspace(0, 1, a["n"]),
                                a["threshold"], codes=True)


def assert_energies_close(got, want, abs_sums):
    finite = np.isfinite(want)
    assert np.array_equal(got[~finite], want[~finite])
    assert (np.abs(got[finite] - want[finite]) <= TOL * abs_sums[finite]).all(), \
        "largest |dE| / sum|phi| = %g" % np.max(np.abs(got[finite] - want[finite]) / abs_sums[finite])


def decided(c):
    """The pairs whose verdict does not hinge on the rounding of the sum: every barrier and the interior maximum stay MARGIN
    away from their ties (BR.margins)."""
    m = np.array([BR.margins(row, c["threshold"]) if np.isfinite(row).all() else (0.0, 0.0) for row in c["energies"]])
    return (m.reshape(-1, 2) >= BR.MARGIN).all(axis=1)


@pytest.mark.parametrize("spec", RAW, ids=lambda s: "%s-rc%.2fh-S%s-n%d-P%d%s" % (s[0], s[1], s[2], s[3], s[4], "-outside" if s[5] else ""))
def test_energies_against_the_restatement(contexts, spec):
    c = raw_case(*spec)
    assert c["n_terms"].max() <= 100000 and c["n_terms"].sum() > 0
    energies, verdict, code = call(contexts(c["cell"]), c)
    assert energies.shape == c["energies"].shape and energies.dtype == np.float64
    print("terms per image: up to %d; largest |dE| / sum|phi| = %g"
          % (c["n_terms"].max(), np.nanmax(np.abs(energies - c["energies"]) / np.where(c["abs_sums"] > 0, c["abs_sums"], np.nan), initial=0.0)))
    assert np.array_equal(code, c["codes"])
    assert_energies_close(energies, c["energies"], c["abs_sums"])
    sure = decided(c)
    assert np.array_equal(verdict[sure], c["verdicts"][sure])
    # the verdict is the header's on the device's own energies, whatever the margins
    assert np.array_equal(verdict, np.array([BR.verdict(row, c["threshold"]) for row in energies], dtype=np.uint8).reshape(-1, 3))


def test_some_path_leaves_the_cell(contexts):
    c = raw_case("cubic", 0.45, 5, 3, 300, False)
    assert (c["codes"] != 111).sum() > 100
    assert len(set(c["codes"].tolist())) > 10


def test_no_pair_touches_nothing(contexts):
    c = raw_case("cubic", 0.45, 5, 3, 0, False)
    ctx = contexts(c["cell"])
    energies, verdict, code = call(ctx, c)
    assert energies.shape == (0, 3) and verdict.shape == (0, 3) and code.shape == (0,)
    # nothing is looked at: not even the arguments that would be refused
    ctx.barrier_energies(np.zeros((0, 3)), [], [], -1.0, c["centers"], np.zeros((0, 2)), [0.0, 1.0], 1.0)


def test_two_calls_give_the_same_bytes(contexts):
    for spec in (("cubic", 0.45, "tile+1", 20, 2, True), ("cubic4", 2.6, 65, 5, 2, True), ("cubic", 0.45, 5, 3, 300, False)):
        c = raw_case(*spec)
        first, second = call(contexts(c["cell"]), c), call(contexts(c["cell"]), c)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        assert first[2].tobytes() == second[2].tobytes()


@pytest.mark.parametrize("spec", [("cubic", 0.45, 65, 67, 2, True), ("triclinic", 0.45, 65, 20, 2, True), ("cubic4", 2.6, 65, 5, 2, True),
                                  ("small_triclinic", 1.4, 3, 5, 2, True)], ids=lambda s: s[0])
def test_whole_cell_shifts_change_nothing(contexts, spec):
    c = raw_case(*spec)
    ctx = contexts(c["cell"])
    rng = np.random.default_rng(3)
    base = call(ctx, c)[0]
    moved_atoms = c["static"] + rng.integers(-3, 4, c["static"].shape).astype(np.float64) @ c["cell"]
    assert_energies_close(call(ctx, c, static=moved_atoms)[0], base, c["abs_sums"])
    # both centres of a pair by the same lattice vector: every pair (k, k + 1) shares it, so all centres move together
    moved_centers = c["centers"] + np.array([2.0, -3.0, 1.0]) @ c["cell"]
    assert_energies_close(call(ctx, c, centers=moved_centers)[0], base, c["abs_sums"])


# ---- the driven points, bit for bit -----------------------------------------------------------------------------------------

def single_term_case():
    """A one-atom lattice with sigma so small that exactly one term contributes at every image: the energy is then one phi of
    one squared distance, and equal bytes mean equal driven points.  The path crosses the cell boundary, so the term's
    translation is not zero."""
    a, b = np.array([11.3, 6.0, 6.0]), np.array([0.8, 6.1, 5.9])
    atom = np.array([0.05, 6.6, 6.2])
    return BR._case(BR.CUBIC, [atom], [a, b], BR._both_ways(2, [(0, 1)]), 1.0, lj_kw={"sigma": 0.45}, n_driven_images=20)


def operator_for(case):
    from sitator_amd import MergeSitesByBarrier
    from sitator_amd.calculators import LennardJones
    return MergeSitesByBarrier(LennardJones(**case["lj"]), **case["kw"])


def trajectory_for(case, n_ij=True, positions=None, centers=None):
    from sitator_amd import SiteNetwork, SiteTrajectory, Structure
    sn = SiteNetwork(Structure(case["positions"] if positions is None else positions, case["cell"], case["numbers"]),
                     case["static_mask"], case["mobile_mask"])
    sn.centers = np.array(case["centers"] if centers is None else centers, copy=True)
    if case["site_types"] is not None:
        sn.site_types = case["site_types"].copy()
    if n_ij:
        sn.add_edge_attribute("n_ij", case["n_ij"].copy())
    return SiteTrajectory(sn, case["traj"].copy())


def run_operator(case, **kw):
    """What a golden case stores, from the operator."""
    op = operator_for(case)
    run_kw = {} if case["coordinating_mask"] is None else {"coordinating_mask": case["coordinating_mask"].copy()}
    out = {"error": "", "op": op}
    try:
        st = op.run(trajectory_for(case, **kw), **run_kw)
        out.update(traj=st.traj, centers=np.asarray(st.site_network.centers), site_types=st.site_network.site_types, st=st)
    except Exception as e:                                       # noqa: BLE001 - compared by class name with the golden
        out["error"] = type(e).__name__
    return out


def test_driven_points_are_the_references_bit_for_bit():
    case = single_term_case()
    want = BR.sites_to_merge(case)
    assert (want["n_terms"] == 1).all() and (want["codes"] != 111).all()
    static_pos, eps, sigma, rc = BR.case_arrays(case)
    triples = np.array([BR.terms(case["cell"], static_pos, eps, sigma, rc, x)[3][0] for x in want["points"][0]])
    assert (triples != 0).any()
    got = run_operator(case)
    assert got["error"] == ""
    assert got["op"].energies_.tobytes() == want["energies"].tobytes()


# ---- the operator against the reference's goldens -------------------------------------------------------------------------

@pytest.mark.parametrize("name", BG.names)
def test_operator_equals_the_reference(name):
    case, exp = BG.case(name), BG.expected(name)
    got = run_operator(case)
    op = got["op"]
    assert got["error"] == exp["error"]
    assert op.pairs_.shape == exp["pairs"].shape and np.array_equal(op.pairs_, exp["pairs"])
    assert op.mergable_.dtype == np.bool_ and np.array_equal(op.mergable_, exp["mergable"])
    assert op.energies_.shape == exp["energies"].shape
    assert_energies_close(op.energies_, exp["energies"], exp["abs_sums"])
    groups = [np.asarray(g) for g in op._get_sites_to_merge(trajectory_for(case),
                                                            **({} if case["coordinating_mask"] is None
                                                               else {"coordinating_mask": case["coordinating_mask"]}))]
    assert len(groups) == len(exp["groups"]) and all(np.array_equal(a, b) for a, b in zip(groups, exp["groups"]))
    if not exp["error"]:
        assert got["traj"].dtype == np.int64 and np.array_equal(got["traj"], exp["traj"])
        assert np.array_equal(got["centers"], exp["centers"])
        if case["kw"].get("check_types"):
            assert np.array_equal(got["site_types"], exp["site_types"])
        else:
            assert got["site_types"] is None


@pytest.mark.parametrize("name", BG.names)
def test_whole_cell_shifts_change_no_golden_verdict(contexts, name):
    case, exp = BG.case(name), BG.expected(name)
    if not len(exp["pairs"]):
        return
    static_pos, eps, sigma, rc = BR.case_arrays(case)
    n, thr = case["kw"].get("n_driven_images", 20), case["kw"]["barrier_threshold"]
    ctx = contexts(case["cell"])
    want = np.array([BR.verdict(row, thr) for row in exp["energies"]], dtype=np.uint8)
    rng = np.random.default_rng(7)
    shifted_atoms = static_pos + rng.integers(-3, 4, static_pos.shape).astype(np.float64) @ case["cell"]
    shifted_centers = case["centers"] + np.array([-2.0, 1.0, 3.0]) @ case["cell"]
    for atoms, centers in ((static_pos, case["centers"]), (shifted_atoms, case["centers"]), (static_pos, shifted_centers)):
        energies, verdict, _ = ctx.barrier_energies(atoms, eps, sigma, rc, centers, exp["pairs"], np.linspace(0, 1, n), thr)
        assert np.array_equal(verdict, want)
        assert_energies_close(energies, exp["energies"], exp["abs_sums"])


def test_without_n_ij_a_jump_analysis_runs_first():
    from sitator_amd import JumpAnalysis
    case = BG.case("chain_of_three")
    plain = trajectory_for(case, n_ij=False)
    JumpAnalysis().run(plain)
    n_ij = np.array(plain.site_network.n_ij, copy=True)
    assert (n_ij > 0).any()
    case = dict(case, n_ij=n_ij)
    with_it, without = run_operator(case), run_operator(case, n_ij=False)
    assert with_it["error"] == without["error"] == ""
    assert without["st"].site_network is not None and np.array_equal(with_it["traj"], without["traj"])
    assert np.array_equal(with_it["centers"], without["centers"])
    assert np.array_equal(with_it["op"].mergable_, without["op"].mergable_)
    assert np.array_equal(with_it["op"].pairs_, without["op"].pairs_) and len(with_it["op"].pairs_) > 0


# ---- what is refused ------------------------------------------------------------------------------------------------------

def test_other_calculators_are_refused():
    from sitator_amd import MergeSitesByBarrier

    class Other(object):
        def get_potential_energy(self, atoms):
            return 0.0
    with pytest.raises(TypeError, match="LennardJones"):
        MergeSitesByBarrier(Other(), 1.0)


def test_two_images_are_refused():
    case = BG.case("low_barrier")
    case["kw"]["n_driven_images"] = 2
    with pytest.raises(AssertionError):
        operator_for(case)


def test_a_coordinating_mask_over_the_mobile_atoms_is_refused():
    case = BG.case("low_barrier")
    with pytest.raises(AssertionError):
        operator_for(case).run(trajectory_for(case), coordinating_mask=np.ones(len(case["positions"]), dtype=bool))


def test_bad_arguments_of_the_entry_point(contexts):
    c = raw_case("cubic", 0.45, 5, 3, 300, False)
    ctx = contexts(c["cell"])
    for bad in (np.array([[0, 301]]), np.array([[-1, 0]])):
        with pytest.raises(ValueError, match="pair index"):
            call(ctx, c, pairs=bad)
    with pytest.raises(ValueError, match="3 driven images"):
        call(ctx, c, n=2)
    with pytest.raises(ValueError, match="epsilon or sigma"):
        call(ctx, c, eps=np.where(np.arange(5) == 3, 0.0, c["eps"]))
    with pytest.raises(ValueError, match="epsilon or sigma"):
        call(ctx, c, sigma=-c["sigma"])
    with pytest.raises(ValueError, match="rc"):
        call(ctx, c, rc=0.0)
    with pytest.raises(ValueError, match="coordinating atom"):
        call(ctx, c, static=np.zeros((0, 3)), eps=[], sigma=[])
    with pytest.raises(ValueError, match="16384"):
        call(ctx, c, centers=np.zeros((16385, 3)))
    # the context still works
    assert_energies_close(call(ctx, c)[0], c["energies"], c["abs_sums"])


def test_lennard_jones_parameters():
    from sitator_amd.calculators import LennardJones
    lj = LennardJones(epsilon={8: 1.0, 16: 0.4}, sigma={8: 1.0, 16: 1.3})
    assert lj.rc == 3.0 * 1.3
    eps, sigma = lj.parameters_for([8, 16, 16])
    assert eps.tolist() == [1.0, 0.4, 0.4] and sigma.tolist() == [1.0, 1.3, 1.3]
    assert LennardJones(sigma=2.0).rc == 6.0 and LennardJones(rc=2.5).rc == 2.5
    for bad in (dict(epsilon=0.0), dict(sigma=-1.0), dict(rc=0.0), dict(epsilon={8: -1.0}), dict(sigma={8: 0.0})):
        with pytest.raises(ValueError):
            LennardJones(**bad)
    with pytest.raises(ValueError, match="atomic number"):
        lj.parameters_for([8, 3])


def test_plan_reports_what_the_kernel_was_built_with():
    from sitator_amd import _lib
    for cell, rc in ((BR.CUBIC, 3.0), (BR.SMALL_TRICLINIC, 4.8), (BR.TRICLINIC, 30.0)):
        plan = _lib.barrier_plan(cell, rc)
        assert np.array_equal(plan["translations"], BR.plan_translations(cell, rc))
        assert plan["tile"] >= 64 and plan["threads"] % 64 == 0 and plan["lds_bytes"] <= 160 * 1024 // 2
    with pytest.raises(ValueError):
        _lib.barrier_plan(np.zeros((3, 3)), 1.0)
    with pytest.raises(ValueError):
        _lib.barrier_plan(BR.CUBIC, -1.0)
